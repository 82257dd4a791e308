"""CPU tier of the leave-one-out cross-validation (include/sigp.h: sigp_loo, sigp_loo_batch, sigp_small_run_loo): the ABI is
declared, exported and bound; the argument checks that need no device; and the closed forms the GPU tests use as their
yardstick for large n, pinned here against REAL oracle refits on n - 1 points."""
import ctypes as C
import os
import re
import types

import numpy as np
import pytest

from oracle import gp_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOO_SYMBOLS = {"sigp_loo": 5, "sigp_loo_batch": 11, "sigp_small_run_loo": 13}


def loo_closed_form(Kt, y, mode="refit"):
    """Rasmussen & Williams 5.4.2 with this engine's profiled signal variance, from the explicit inverse of K~:
    g_i = [K~^-1]_ii, mean_i = y_i - A~_i / g_i, var_i = s_i / g_i with s_i = (q - A~_i^2 / g_i) / (n - 1) ("refit") or q / n ("fixed")."""
    y = np.asarray(y, dtype=np.float64).reshape(-1)
    n = len(y)
    Ki = np.linalg.inv(Kt)
    A = Ki @ y
    g = np.diag(Ki).copy()
    q = float(y @ A)
    mean = y - A / g
    sf_loo = (q - A * A / g) / (n - 1) if mode == "refit" else np.full(n, q / n)
    var = sf_loo / g
    r = y - mean
    return dict(mean=mean, var=var, sigma_f=sf_loo, nlpd=float(np.sum(0.5 * np.log(2 * np.pi * var) + r * r / (2 * var))), sse=float(np.sum(r * r)))


def oracle_refits(X, y, ell, sn, kind, M=None):
    """fit on the other n - 1 points, predict the left-out one -- for every point (M, like the features, stays the full set's)"""
    n = len(y)
    mean, var, sf = np.zeros(n), np.zeros(n), np.zeros(n)
    for i in range(n):
        k = np.arange(n) != i
        r = O.fit_predict(X[k], y[k], X[i:i + 1], ell, sn, kind=kind, M=M, ref_idiom=False)
        mean[i], var[i], sf[i] = r["fmean"][0], r["fvar"][0], r["sigma_f"]
    return mean, var, sf


def test_loo_entry_points_declared_exported_and_bound():
    from seaiceextentforecasting_amd import _lib as L
    hdr = open(os.path.join(ROOT, "include", "sigp.h")).read()
    lib = C.CDLL(L.LIB_PATH)
    for name, nargs in LOO_SYMBOLS.items():
        m = re.search(r"\bint\s+%s\s*\(([^;]*?)\)\s*;" % name, hdr, re.S)
        assert m, "%s is not declared in include/sigp.h" % name
        assert len(m.group(1).split(",")) == nargs, (name, m.group(1))
        assert hasattr(lib, name), "%s is not exported by libsigp.so" % name
        assert name in L.SIGNATURES and len(L.SIGNATURES[name][1]) == nargs, name
    assert re.search(r"SIGP_LOO_REFIT\s*=\s*0\s*,\s*SIGP_LOO_FIXED\s*=\s*1", hdr)
    assert L.load().sigp_version() >= 510
    assert L.LOO_MODES == {"refit": 0, "fixed": 1}


def test_loo_null_handle_and_null_buffers_are_rejected_before_any_device_work():
    from seaiceextentforecasting_amd import _lib as L
    lib = L.load()
    a = np.zeros(4)
    i64 = np.zeros(1, dtype=np.int64)
    assert lib.sigp_loo(None, 0, L.ptr(a), L.ptr(a), L.ptr(a)) == L.BAD_ARG
    assert lib.sigp_loo(None, 0, None, None, None) == L.BAD_ARG
    assert lib.sigp_loo_batch(None, 0, 1, 1, L.ptr(a), L.ptr(a), 0, None, None, 0, L.ptr(a)) == L.BAD_ARG
    assert lib.sigp_small_run_loo(None, 1, L.iptr(i64), L.ptr(a), L.ptr(a), 0, L.ptr(a), None, None, 0, L.ptr(a), L.ptr(a), 4) == L.BAD_ARG
    assert lib.sigp_small_run_loo(None, 1, L.iptr(i64), L.ptr(a), L.ptr(a), 7, L.ptr(a), None, None, 0, L.ptr(a), L.ptr(a), 4) == L.BAD_ARG


def test_python_argument_checks_need_no_device():
    import seaiceextentforecasting_amd as S
    from seaiceextentforecasting_amd.retro import retro_grid_search
    for name in ("loo", "loo_batch", "loo_grid"):
        assert callable(getattr(S.GPR, name, None)), name
    with pytest.raises(ValueError):
        retro_grid_search("September1st", {}, {}, 2000, 2001, criterion="bogus")
    sb = S.SmallBatch(types.SimpleNamespace(kernel="netdiffusion", dtype="f64"))
    with pytest.raises(ValueError):
        sb.run(loo="bogus")
    with pytest.raises(ValueError):
        sb.run(grad=True, loo="refit")


@pytest.mark.parametrize("kind,n,d,ell,seed", [("rbf", 64, 8, np.sqrt(8.0), 11), ("rbf", 300, 8, np.sqrt(8.0), 12), ("matern52", 200, 8, np.sqrt(8.0), 13),
                                               ("netdiffusion", 25, 12, 0.05, 14), ("netdiffusion", 40, 12, 0.05, 15)])
def test_closed_forms_equal_real_oracle_refits(kind, n, d, ell, seed):
    """The yardstick of the GPU tests: the closed forms from inv(K~) == n real fits on n - 1 points, to 1e-10."""
    X, y, _ = O.synthetic_problem(n, d, seed)
    sn = 1e-2
    M = O.laplacian_M(X) if kind == "netdiffusion" else None
    Kt = O.fit_predict(X, y, X[:1], ell, sn, kind=kind, M=M, ref_idiom=False)["K_tilde"]
    cf = loo_closed_form(Kt, y, "refit")
    mean, var, sf = oracle_refits(X, y, ell, sn, kind, M)
    print("cond(K~) %.3g  mean %.3g  var %.3g  sigma_f %.3g" % (np.linalg.cond(Kt), np.max(np.abs(cf["mean"] - mean)) / np.max(np.abs(y)),
                                                              np.max(np.abs(cf["var"] / var - 1)), np.max(np.abs(cf["sigma_f"] / sf - 1))))
    assert np.max(np.abs(cf["mean"] - mean)) <= 1e-10 * np.max(np.abs(y))
    assert np.max(np.abs(cf["var"] / var - 1)) <= 1e-10
    assert np.max(np.abs(cf["sigma_f"] / sf - 1)) <= 1e-10
    # "fixed" differs from "refit" by the signal variance alone
    fx = loo_closed_form(Kt, y, "fixed")
    assert np.array_equal(fx["mean"], cf["mean"]) and np.allclose(fx["var"] / cf["var"], fx["sigma_f"] / cf["sigma_f"], rtol=1e-13, atol=0)
